"""TEST HELPER: plain numpy model of one rerank of the L-first path -- lf_rerank() of csrc/lfirst.inc and the classification behind it, what
dk_dbg_dev_lf_rerank runs -- written from the rules below over the WHOLE list, with no tiles, waves or stretches in it.
tests/test_lf_rerank_model.py pins it against a per-slot Python loop and against `brute` of tests/test_lfirst_logic.py before
tests/test_gpu_lfirst_layer.py lets it judge the device.  Integers only, no tolerance anywhere.

The input is a list of `count` SLOTS in sorted order: keys[a], the suffix idx[a], the symbol sym[a] in front of that suffix, and in a LATER
rerank the SA position pos_in[a].  In the FIRST rerank (pos_in None) slot a is SA position a.

Heads.  Slot a is a HEAD if a == 0, or the compared key bits change there -- 8-byte keys: keys[a] >> cmp_shift != keys[a - 1] >> cmp_shift;
4-byte keys: the words differ -- or (4-byte keys with 256 bucket starts) a is one of the bucket starts; a start from `count` up names no slot.
A GROUP is the run of slots from a head up to the next one.

Symbols.  With sym_from_key (8-byte keys) a slot's symbol is keys[a] & 0xFF, and the sym array holds those bytes for every slot afterwards;
otherwise it is sym[a] and the array stays as it is.

Live.  A group is LIVE iff it has more than one member and a REASON: two different symbols in front among its members, or suffix 0 among
them.  Suffix 0 stands in slot zero_slot where that is given (a value from `count` up: in no slot) and in the slots with idx[a] == 0
otherwise.  Every slot of a group that is not live is FINAL -- singletons (suffix 0 in a singleton too) and groups of one symbol in front.

Active list.  The live slots in slot order: out_idx = idx[a], out_pos = pos_in[a] (first rerank: a), out_gid = the number of live groups in
front of a's group, out_sym = a's symbol.  active = its length, groups = the live groups.  gstart[g] = the place of group g's head in the
list for g < groups, and the scan writes gstart[groups] = active behind the last group.

Depths.  gdepth[g] for g < groups (where the caller passes the table): `depth` for every group, or by the big-list rule
bigdepth[keys[head slot of g] >> key_shift] + depth_add.  (The rule's token fields are not modelled: the entry leaves them out.)

Finals.  Later reranks only: bwt[pos_in[a]] = a's symbol for every final slot, and origin = pos_in[a] for the final slot with idx[a] == 0.
The first rerank writes nothing into L or the origin word: its finals stand in L already.

Classification of the live groups by size: a group of more than ls_max members (LFS_CAP = 256) is BIG; big_groups and big_slots count them
and their members.

Everything else stays as it was: the lists from `active` on, gstart from groups + 1 on, gdepth from `groups` on, bwt at the positions of live
slots, the origin word unless suffix 0 is final.  apply_model() lays the model's values over what the arrays held before, so that a
comparison of whole arrays says that too."""
from types import SimpleNamespace

import numpy as np

TILE = 2048         # RR_TILE: slots per tile of k_lf_reduce / k_lf_apply
STRADDLE_WAVE = 64  # tiles one round of k_lf_straddle's loop looks at
SCAN_CHUNK = 1024   # RSC_CHUNK: tiles per chunk of the three-phase scan, which runs above 4 * SCAN_CHUNK tiles
LS_MAX = 256        # LFS_CAP: the line of the big groups behind the path's first rerank
COUNT_NAMES = ("active", "groups", "big_slots", "big_groups")


def lf_heads(keys, cmp_shift=0, bucket_starts=None):
    keys = np.asarray(keys)
    n = len(keys)
    k = keys if keys.dtype == np.uint32 else keys.astype(np.uint64) >> np.uint64(cmp_shift)
    head = np.zeros(n, bool)
    head[0] = True
    head[1:] = k[1:] != k[:-1]
    if bucket_starts is not None:
        s = np.asarray(bucket_starts, dtype=np.int64)
        head[s[s < n]] = True
    return head


def lf_rerank_model(keys, idx, sym=None, pos_in=None, bucket_starts=None, cmp_shift=0, sym_from_key=False, zero_slot=None, depth=None,
                    bigdepth=None, key_shift=0, depth_add=0, ls_max=LS_MAX):
    """-> namespace: active, groups, out_idx / out_pos / out_gid / out_sym (active entries), gstart (groups + 1), gdepth (groups entries or None),
    live (boolean per slot), head, final (slots), final_pos, final_sym, origin (None: not written), sym_after (None: the array stays),
    big_groups, big_slots, counts"""
    keys = np.asarray(keys)
    idx = np.asarray(idx, dtype=np.uint32)
    n = len(idx)
    first = pos_in is None
    slots = np.arange(n, dtype=np.int64)
    head = lf_heads(keys, cmp_shift, bucket_starts)
    s = (keys.astype(np.uint64) & np.uint64(0xFF)).astype(np.uint8) if sym_from_key else np.asarray(sym, dtype=np.uint8)
    starts = np.flatnonzero(head)
    sizes = np.diff(np.append(starts, n))
    group_of = np.cumsum(head) - 1
    reason = np.zeros(len(starts), bool)
    reason[group_of[s != s[starts][group_of]]] = True                       # a member whose symbol is not its head's: two symbols in front
    zero = np.flatnonzero(idx == 0) if zero_slot is None else np.array([zero_slot] if zero_slot < n else [], np.int64)
    reason[group_of[zero]] = True
    live_group = (sizes > 1) & reason
    live = np.repeat(live_group, sizes)
    act = np.flatnonzero(live)
    pos = slots.astype(np.uint32) if first else np.asarray(pos_in, dtype=np.uint32)
    m = SimpleNamespace(first=first, active=len(act), groups=int(live_group.sum()), head=head, live=live)
    m.out_idx, m.out_pos, m.out_sym = idx[act], pos[act], s[act]
    m.out_gid = (np.cumsum(head & live)[act] - 1).astype(np.uint32)
    live_heads = starts[live_group]
    m.gstart = np.append(np.searchsorted(act, live_heads), len(act)).astype(np.uint32)
    m.gdepth = None
    if bigdepth is not None:
        m.gdepth = (np.asarray(bigdepth, dtype=np.uint32)[(keys[live_heads].astype(np.uint64) >> np.uint64(key_shift)).astype(np.int64)]
                    + np.uint32(depth_add)).astype(np.uint32)
    elif depth is not None:
        m.gdepth = np.full(m.groups, depth, np.uint32)
    m.final = np.flatnonzero(~live)
    m.final_pos, m.final_sym = pos[m.final], s[m.final]
    m.origin = None
    if not first:
        z = m.final[idx[m.final] == 0]
        if len(z):
            m.origin = int(pos[z[0]])
    m.sym_after = s if sym_from_key else None
    gsz = np.diff(m.gstart.astype(np.int64))
    m.big_groups, m.big_slots = int((gsz > ls_max).sum()), int(gsz[gsz > ls_max].sum())
    m.counts = (m.active, m.groups, m.big_slots, m.big_groups)
    return m


def apply_model(m, before):
    """before: {name: array or None} of out_idx, out_pos, out_gid, out_sym, gstart, gdepth, sym, bwt and origin (an int or None) as they are
    before the call -> the same after it.  Entries of pos_in are distinct (the path's own lists are), so no two stores of the model meet."""
    after = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in before.items()}
    for name in ("out_idx", "out_pos", "out_gid", "out_sym"):
        after[name][:m.active] = getattr(m, name)
    after["gstart"][:m.groups + 1] = m.gstart
    if after.get("gdepth") is not None:
        after["gdepth"][:m.groups] = m.gdepth
    if m.sym_after is not None:
        after["sym"][:] = m.sym_after
    if not m.first:
        after["bwt"][m.final_pos] = m.final_sym
        if m.origin is not None:
            after["origin"] = m.origin
    return after


# ---- the same, one slot at a time (tests/test_lf_rerank_model.py compares the two) --------------------------------------------------------------
def lf_rerank_loop(keys, idx, sym=None, pos_in=None, bucket_starts=None, cmp_shift=0, sym_from_key=False, zero_slot=None, depth=None,
                   bigdepth=None, key_shift=0, depth_add=0, ls_max=LS_MAX):
    """-> dict of plain lists and numbers under lf_rerank_model's names, straight from the sentences of the module docstring"""
    n = len(idx)
    first = pos_in is None
    narrow = np.asarray(keys).dtype == np.uint32
    forced = set(int(x) for x in bucket_starts) if bucket_starts is not None else set()
    cmp = [int(k) if narrow else int(k) >> cmp_shift for k in keys]
    s = [int(k) & 0xFF for k in keys] if sym_from_key else [int(x) for x in sym]
    r = dict(out_idx=[], out_pos=[], out_gid=[], out_sym=[], gstart=[], gdepth=[], bwt={}, origin=None, live=[False] * n, big_slots=0, big_groups=0)
    a = 0
    while a < n:
        b = a + 1
        while b < n and not (cmp[b] != cmp[b - 1] or b in forced):
            b += 1
        has_zero = (a <= zero_slot < b) if zero_slot is not None else any(int(idx[x]) == 0 for x in range(a, b))
        if b - a > 1 and (len(set(s[a:b])) > 1 or has_zero):
            r["gstart"].append(len(r["out_idx"]))
            r["gdepth"].append(depth if bigdepth is None else int(bigdepth[int(keys[a]) >> key_shift]) + depth_add)
            for x in range(a, b):
                r["live"][x] = True
                r["out_idx"].append(int(idx[x]))
                r["out_pos"].append(x if first else int(pos_in[x]))
                r["out_gid"].append(len(r["gstart"]) - 1)
                r["out_sym"].append(s[x])
            if b - a > ls_max:
                r["big_slots"] += b - a
                r["big_groups"] += 1
        elif not first:
            for x in range(a, b):
                r["bwt"][int(pos_in[x])] = s[x]
                if int(idx[x]) == 0:
                    r["origin"] = int(pos_in[x])
        a = b
    r["active"], r["groups"] = len(r["out_idx"]), len(r["gstart"])
    r["gstart"].append(r["active"])
    return r
