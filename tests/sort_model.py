"""TEST HELPER: plain numpy models of what the sort layer (csrc/radix_sort.hip) owes its callers, written from the contracts in
include/dark_amd.h and csrc/context.hpp.  They share no code with the kernels; tests/test_sort_model.py pins each of them against a naive
pure-Python loop before tests/test_gpu_sort_layer.py lets them judge the device paths.  Integers only, no tolerance anywhere.

The order of a sort on bits [lo, hi) is the STABLE order by the field (key >> lo) & (2^(hi - lo) - 1) and by nothing else: what a key holds
below lo or from hi up travels with its pair.  lo >= hi is an empty field: nothing moves."""
import numpy as np

TILE = 8192            # pairs one workgroup sorts inside LDS: the local sort's tile and the largest group sort_groups takes
MARK = 0x80000000      # inverse permutation: bit 31 of an entry = "take the value from marked_val"


def field(keys, lo, hi):
    """the bits [lo, hi) of every key as a number (uint64; zeros for an empty range)"""
    keys = np.asarray(keys, dtype=np.uint64)
    w = hi - lo
    if w <= 0:
        return np.zeros(len(keys), dtype=np.uint64)
    if not (0 <= lo and hi <= 64):
        raise ValueError("bits [%d, %d) outside a 64-bit key" % (lo, hi))
    f = keys >> np.uint64(lo)
    if w < 64:
        f = f & np.uint64((1 << w) - 1)
    return f


def stable_order(keys, lo, hi):
    """the permutation a stable sort on bits [lo, hi) applies: out[i] = in[order[i]]"""
    f = field(keys, lo, hi)
    if hi - lo <= 16:
        f = f.astype(np.uint16)  # (same order; numpy sorts 16-bit words by counting, which keeps the large cases short)
    return np.argsort(f, kind="stable")


def sort_pairs_model(keys, vals, lo, hi):
    """-> (keys, vals) in stable order by bits [lo, hi); the keys come back whole"""
    keys = np.asarray(keys, dtype=np.uint64)
    vals = np.asarray(vals, dtype=np.uint32)
    order = stable_order(keys, lo, hi)
    return keys[order], vals[order]


def local_sort_model(keys, vals, lo, hi, tile=TILE):
    """the same for every tile of `tile` consecutive pairs by itself (the last one may be short)"""
    keys = np.array(keys, dtype=np.uint64)
    vals = np.array(vals, dtype=np.uint32)
    for b in range(0, len(keys), tile):
        keys[b:b + tile], vals[b:b + tile] = sort_pairs_model(keys[b:b + tile], vals[b:b + tile], lo, hi)
    return keys, vals


def sort_groups_model(kin, vin, kout_before, vout_before, starts, above, lo, hi):
    """group g = the pairs [starts[g], starts[g + 1]): a group of more than `above` and at most TILE pairs goes, sorted, to the same places
    of the output; every other place of the output keeps what it held before (in place: pass kin / vin as the output's state before)"""
    kin = np.asarray(kin, dtype=np.uint64)
    vin = np.asarray(vin, dtype=np.uint32)
    kout = np.array(kout_before, dtype=np.uint64)
    vout = np.array(vout_before, dtype=np.uint32)
    starts = [int(s) for s in starts]
    for a, b in zip(starts[:-1], starts[1:]):
        if above < b - a <= TILE:
            kout[a:b], vout[a:b] = sort_pairs_model(kin[a:b], vin[a:b], lo, hi)
    return kout, vout


def inverse_permutation_model(sa, marked_val=None):
    """rank[sa[p] & 0x7FFFFFFF] = marked_val[p] if sa[p] >> 31 else p, for a permutation (marks aside) of 0 .. n-1"""
    sa = np.asarray(sa, dtype=np.uint32)
    n = len(sa)
    marked = (sa & np.uint32(MARK)) != 0
    if marked_val is None and marked.any():
        raise ValueError("marked entries without values for them")
    at = (sa & np.uint32(MARK - 1)).astype(np.int64)
    if n and (int(at.max()) >= n or not (np.bincount(at, minlength=n) == 1).all()):
        raise ValueError("not a permutation of 0 .. %d" % (n - 1))
    val = np.arange(n, dtype=np.uint32)
    if marked_val is not None:
        val[marked] = np.asarray(marked_val, dtype=np.uint32)[marked]
    rank = np.empty(n, dtype=np.uint32)
    rank[at] = val
    return rank
