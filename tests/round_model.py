"""TEST HELPER: plain numpy model of one general round of the suffix sort -- general_round() of csrc/suffix_array.hip, what dk_dbg_dev_round runs --
written from the definition below and not from the kernels.  tests/test_round_model.py pins it against per-suffix Python loops before
tests/test_gpu_round.py lets it judge the device.  Integers only, no tolerance anywhere.

The input is a list of `count` slots: the suffix idx[a], its SA position pos[a], its group gid[a]; group g holds the slots gstart[g] .. gstart[g + 1] - 1
and its members are equal in their first h symbols (h is cut to n).  A round sorts the members of every group, inside the group's own slots, by a
SECONDARY KEY, ties in slot order; the regrouping behind it is tests/rerank_model.py's.

The secondary key of suffix x, one of four forms:
  rank     rank[x + h] + h if x + h < n, else n + h - 1 - (x + h): a suffix that ends inside the next h symbols sorts by "shorter first" and in
           front of every suffix that goes on.  kbits = the bits that hold n + h
  coded    (tsym > 0, at most 16 byte values in the text) the codes of T[x + h .. x + h + tsym), `bits` each, big-endian, zero behind the text's end;
           code[c] = the byte values below c that occur, bits = the bits that hold the largest code (one at least), tsym at most 63 // bits.
           kbits = tsym * bits
  raw      (tsym > 0, 17 byte values or more; and every text key of a token round) the eight bytes T[x + h .. x + h + 8) big-endian, zero behind
           the end.  kbits = 64
  token    (period p > 0, for a suffix of at least h symbols whose stretch of period p covers them: nb[x] - x + p >= h) with b = nb[x], e = b - x,
           brk = b + p, down = brk >= n or T[brk] < T[b], ebits = the bits that hold n:
               bit 63: 0 if down else 1 | ebits bits below it: e if down else 2^ebits - 1 - e | 32 bits below them: T[brk .. brk + 4) big-endian
           -- tests/test_period_tokens.py's token() in the kernel's bit layout.  Every other suffix of a token round takes the raw key.  kbits = 64

A group of more than 1024 members is BIG.  Its members are sorted by the leading kb bits of the secondary key only, and the key the round leaves for
them is (the number of big groups in front of theirs) << kb | those kb bits:
  rank     kb = kbits
  text     kb = tbits * min(tsym, (63 - bsbits) // tbits, max(1, 32 // tbits)) with tbits = 8 (raw) or `bits`, bsbits = the bits that number the big
           groups (one at least).  The round advances the depth by kb // tbits symbols when it has a big group, by tsym otherwise
  token    kb = 1 + ebits + 8: down to the first byte behind the break (for every n below 2^40).  The depth stays
The key left for a member of a small group is its secondary key."""
from types import SimpleNamespace

import numpy as np

import rerank_model as R
from test_period_tokens import next_break as next_break_loop, token as token_loop  # noqa: F401  (the definition the token form restates)

LS_MAX = 1024
TILE = 2048  # LS_TILE: slots per workgroup of k_round_local


def bits_for(v):
    """the smallest b with 2^b >= v"""
    b = 0
    while (1 << b) < v:
        b += 1
    return b


def alphabet(text):
    """-> (code table of 256 entries, sigma, bits per coded symbol)"""
    present = np.zeros(256, bool)
    present[np.unique(text)] = True
    code = (np.cumsum(present) - present).astype(np.uint8)
    sigma = int(present.sum())
    return code, sigma, max(1, bits_for(sigma))


def bytes_be(text, p, count):
    """T[p .. p + count) per entry of p as one big-endian integer, zero behind the text's end (count <= 8)"""
    n = len(text)
    padded = np.concatenate([text, np.zeros(count, np.uint8)]).astype(np.uint64)
    key = np.zeros(len(p), np.uint64)
    for j in range(count):
        key = (key << np.uint64(8)) | padded[np.minimum(p + j, n)]
    return key


def key_rank(rank, idx, n, h):
    p = idx.astype(np.int64) + h
    return np.where(p < n, rank[np.minimum(p, n - 1)].astype(np.int64) + h, n + h - 1 - p).astype(np.uint64)


def key_coded(text, code, bits, tsym, idx, h):
    n = len(text)
    coded = np.concatenate([code[text], np.zeros(1, np.uint8)]).astype(np.uint64)
    p = idx.astype(np.int64) + h
    key = np.zeros(len(idx), np.uint64)
    for j in range(tsym):
        key = (key << np.uint64(bits)) | coded[np.minimum(p + j, n)]
    return key


def key_raw(text, idx, h):
    return bytes_be(text, idx.astype(np.int64) + h, 8)


def periodic(nb, period, idx, n, h):
    """which suffixes take the token: at least h symbols long, and following the period through them"""
    x = idx.astype(np.int64)
    return (x + h <= n) & (nb[x].astype(np.int64) - x + period >= h)


def key_token(text, nb, period, idx):
    n = len(text)
    ebits = bits_for(n + 1)
    x = idx.astype(np.int64)
    b = nb[x].astype(np.int64)
    e = b - x
    brk = b + period
    down = (brk >= n) | (text[np.minimum(brk, n - 1)] < text[np.minimum(b, n - 1)])
    ev = np.where(down, e, (1 << ebits) - 1 - e).astype(np.uint64)
    tail = bytes_be(text, brk, 4)
    return (np.where(down, 0, 1).astype(np.uint64) << np.uint64(63)) | (ev << np.uint64(63 - ebits)) | (tail << np.uint64(31 - ebits))


def plan(n, h, big_groups, tsym, period, sigma_bits, sigma):
    """-> namespace: form ("rank", "coded", "raw", "token"), tsym, kbits, kb, bsbits, advanced_small, advanced_big"""
    bsbits = max(1, bits_for(big_groups))
    if period > 0:
        return SimpleNamespace(form="token", tsym=8, kbits=64, kb=1 + bits_for(n + 1) + 8, bsbits=bsbits, advanced_small=0, advanced_big=0)
    if tsym == 0:
        kbits = bits_for(n + min(h, n))
        return SimpleNamespace(form="rank", tsym=0, kbits=kbits, kb=kbits, bsbits=bsbits, advanced_small=0, advanced_big=0)
    raw = sigma >= 17
    tbits = 8 if raw else sigma_bits
    tsym = 8 if raw else min(tsym, 63 // tbits)
    big = min(tsym, (63 - bsbits) // tbits, max(1, 32 // tbits))
    return SimpleNamespace(form="raw" if raw else "coded", tsym=tsym, kbits=tsym * tbits, kb=big * tbits, bsbits=bsbits, advanced_small=tsym, advanced_big=big)


def secondary_keys(text, h, idx, rank, pl, period=0, nb=None):
    n = len(text)
    h = min(h, n)
    if pl.form == "rank":
        return key_rank(rank, idx, n, h)
    if pl.form == "coded":
        code, _, bits = alphabet(text)
        return key_coded(text, code, bits, pl.tsym, idx, h)
    key = key_raw(text, idx, h)
    if pl.form == "token":
        tok = periodic(nb, period, idx, n, h)
        key[tok] = key_token(text, nb, period, idx[tok])
    return key


def round_model(text, h, idx, pos, gid, gstart, rank=None, tsym=0, period=0, nb=None, sym=None, bwt=None):
    """-> namespace: plan, second (the secondary key per slot of the input), big (per slot: its group is big), order (slot of the input list that
    slot a of the sorted state holds), sorted_keys / sorted_idx / sorted_sym, rr (rerank_model's namespace for the regrouping), advanced"""
    text = np.asarray(text, dtype=np.uint8)
    n = len(text)
    idx, pos, gid, gstart = (np.asarray(a, dtype=np.uint32) for a in (idx, pos, gid, gstart))
    count = len(idx)
    sizes = np.diff(gstart.astype(np.int64))
    big_group = sizes > LS_MAX
    _, sigma, sbits = alphabet(text)
    pl = plan(n, h, int(big_group.sum()), tsym, period, sbits, sigma)
    second = secondary_keys(text, h, idx, rank, pl, period, nb)
    big = big_group[gid]
    dense = (np.cumsum(big_group) - big_group)[gid].astype(np.uint64)  # the big groups in front of the slot's group
    left = np.where(big, (dense << np.uint64(pl.kb)) | (second >> np.uint64(pl.kbits - pl.kb)), second)
    order = np.lexsort((np.arange(count), left, gid))  # inside every group by key, ties in slot order (the groups stand in slot order already)
    m = SimpleNamespace(plan=pl, second=second, big=big, order=order, sorted_keys=left[order], sorted_idx=idx[order], sorted_sym=None if sym is None else np.asarray(sym, np.uint8)[order])
    m.rr = R.rerank_model(m.sorted_keys, m.sorted_idx, pos_in=pos, gid_in=gid, sym_in=m.sorted_sym, bwt=bwt)
    m.advanced = pl.advanced_big if big.any() else pl.advanced_small
    return m


def sound(sorted_keys, sorted_idx, gid, isa):
    """the check that needs no model of the keys: inside every old group the new groups (runs of one key) stand in true suffix order -- every
    member of one is smaller than every member of the next.  isa: the text's inverse suffix array.  -> the borders between new groups looked at"""
    gid = np.asarray(gid)
    r = isa[np.asarray(sorted_idx)].astype(np.int64)
    head, _ = R.heads_model(sorted_keys, gid)
    starts = np.flatnonzero(head)
    lo, hi = np.minimum.reduceat(r, starts), np.maximum.reduceat(r, starts)
    inside = gid[starts[1:]] == gid[starts[:-1]]  # a border between two new groups of one old group
    bad = np.flatnonzero(inside & (hi[:-1] >= lo[1:]))
    assert not len(bad), "new groups out of suffix order: the one at slot %d and the next" % starts[bad[0]]
    return int(inside.sum())
